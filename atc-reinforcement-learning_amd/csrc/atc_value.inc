// atc_value.inc — the critic in the library (include/atc_step.h: atc_value_forward, atc_ppo_value_grad): k_value_forward<KT>,
// k_ppo_value_grad<KT> and k_ppo_value_grad_reduce.  Included by atc_step.hip behind atc_ppo_grad.inc.
//   THE CRITIC is the policy's trunk with one output: (10 + 7 K) -> 64 -> 64 -> 1, tanh, packed like the policy without its two further head
//   rows and without log_std (ValOff).  Both kernels evaluate it in policy_decide's arithmetic and operation order: the fmaf chain of layer 1
//   over the inputs — in float64 where the WAVEFRONT holds an input above 4 in magnitude —, layer 2 in four partial sums, and the head
//   v = b3; v = fmaf(W3[j], h2_j, v) for j = 0 .. 63 inside layer 2's loop.  Weights through the constant address space at wave-uniform
//   indices (scalar loads).  The two kernels share no device function (k_value_forward keeps h1 in registers and h2 nowhere,
//   k_ppo_value_grad stages both in LDS) but every operation of a row's v is the same in both, and the file is built with
//   -ffp-contract=off: 64 consecutive rows give the same bits in both.
//   k_value_forward: LANE = ROW, 256 rows per workgroup, no LDS, no activation in memory.
//   k_ppo_value_grad: k_ppo_grad's structure (atc_ppo_grad.inc, MAPPING .. DETERMINISM there) with the critic's head: one dv word per row
//   where the policy has three dmu and three dlog_std, so the stage `dms` holds dv during a tile and the eight statistics at the end.  The
//   text of the trunk (hidden-layer forward, backward through both tanh layers, dW2 / dW1 accumulation) is a copy of k_ppo_grad's, which
//   is left byte for byte as it was (DESIGN.md section 3p).
template <int IN>
struct ValOff {
    enum { W1 = 0, B1 = ATC_POLICY_HIDDEN * IN, W2 = B1 + ATC_POLICY_HIDDEN, B2 = W2 + ATC_POLICY_HIDDEN * ATC_POLICY_HIDDEN, W3 = B2 + ATC_POLICY_HIDDEN,
           B3 = W3 + ATC_POLICY_HIDDEN, WORDS = B3 + 1 };
};
static_assert(ValOff<ATC_POLICY_TRAFFIC_IN(0)>::WORDS == ATC_VALUE_WORDS(0) && ValOff<ATC_POLICY_TRAFFIC_IN(1)>::WORDS == ATC_VALUE_WORDS(1) &&
              ValOff<ATC_POLICY_TRAFFIC_IN(2)>::WORDS == ATC_VALUE_WORDS(2) && ValOff<ATC_POLICY_TRAFFIC_IN(4)>::WORDS == ATC_VALUE_WORDS(4) &&
              ATC_VALUE_WORDS(0) == 4929 && ATC_VALUE_WORDS(1) == 5377 && ATC_VALUE_WORDS(2) == 5825 && ATC_VALUE_WORDS(4) == 6721, "the packed critic's layout");
static_assert(ATC_PPO_VALUE_STATS == ATC_PPO_GRAD_STATS, "scratch rows of both gradient calls carry eight statistics");

constexpr int kValueBlock = 256;
// wavefronts per SIMD k_value_forward is register-budgeted for: 3 (<= 168 VGPRs; it takes 133) like k_rollout_policy — 64 h1 words and
// the input row are live through layer 1 (133 - 144 taken); at 4 (<= 128) every K spills 28 - 84 bytes per lane —, and 2 with K = 4: its 38
// inputs in float32 and float64 next to h1 take 186 registers, and within 168 the compiler spills 1 236 scalar and 448 vector words.  -DATC_VALUE_WAVES=n: A/B builds.
#ifndef ATC_VALUE_WAVES
#define ATC_VALUE_WAVES 3
#endif

template <int KT>
__global__ void __launch_bounds__(kValueBlock, KT == 4 && ATC_VALUE_WAVES > 2 ? 2 : ATC_VALUE_WAVES)
k_value_forward(int R, const float* __restrict__ w_arg, const float* __restrict__ xin, float* __restrict__ values) {
    constexpr int IN = ATC_POLICY_TRAFFIC_IN(KT), H = ATC_POLICY_HIDDEN;
    typedef ValOff<IN> O;
    pol_wptr w = (pol_wptr)(uintptr_t)w_arg;
    const long long i = (long long)blockIdx.x * kValueBlock + threadIdx.x;
    const bool have = i < (long long)R;
    float x[IN];
#pragma unroll
    for (int c = 0; c < IN; ++c) x[c] = 0.0f;
    if (have) {
        const float* o = xin + (size_t)i * IN;
#pragma unroll
        for (int c = 0; c < IN; ++c) x[c] = o[c];
    }
    float h1[H];
    float xmax = 0.0f;
#pragma unroll
    for (int c = 0; c < IN; ++c) xmax = fmaxf(xmax, fabsf(x[c]));
    if (ATC_RARE(__builtin_amdgcn_ballot_w64(!(xmax <= 4.0f)) != 0ull)) {
#pragma unroll
        for (int j = 0; j < H; ++j) {
            double s = (double)w[O::B1 + j];
#pragma unroll
            for (int c = 0; c < IN; ++c) s = __builtin_fma((double)w[O::W1 + j * IN + c], (double)x[c], s);
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
    for (int j = 0; j < H; ++j) h1[j] = tanhf(h1[j]);
    float v = w[O::B3];
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
        v = fmaf(w[O::W3 + j], h2, v);
    }
    if (have) values[i] = v;
}

template <int KT>
__global__ void __launch_bounds__(kPpoBlock)
k_ppo_value_grad(int R_src, int R, const float* __restrict__ w_arg, const float* __restrict__ obs_rows, const float* __restrict__ traffic,
                 const float* __restrict__ v_old, const float* __restrict__ ret, const uint8_t* __restrict__ mask, const int32_t* __restrict__ index,
                 float clip, float* __restrict__ value, float* __restrict__ scratch) {
    constexpr int IN = ATC_POLICY_TRAFFIC_IN(KT), H = ATC_POLICY_HIDDEN, S = kPpoStride;
    typedef ValOff<IN> O;
    __shared__ float xs[IN * S], h1s[H * S], h2s[H * S], dms[ATC_PPO_VALUE_STATS * S];
    const int lane = threadIdx.x;
    float aW1[IN], aW2[H], aW3 = 0.0f, ab1 = 0.0f, ab2 = 0.0f, ab3 = 0.0f;
#pragma unroll
    for (int c = 0; c < IN; ++c) aW1[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < H; ++c) aW2[c] = 0.0f;
    uint32_t n_part = 0u, n_cut = 0u;
    float sum_l = 0.0f, sum_v = 0.0f, sum_ret = 0.0f, sum_ret2 = 0.0f, sum_err2 = 0.0f, max_dv = 0.0f;
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

        float x[IN], vo = 0.0f, rt = 0.0f;
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
            vo = v_old[src];
            rt = ret[src];
        }
        ppo_lds_order();                    // (the tile before this one has read its stages)
#pragma unroll
        for (int c = 0; c < IN; ++c) xs[c * S + lane] = x[c];

        // ---- forward: k_value_forward's, with h1 and h2 kept ----
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
        float v = w[O::B3];
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
            v = fmaf(w[O::W3 + j], h2, v);
        }

        // ---- the clipped value loss of the row and dL/dv ----
        const float e = v - rt, dlt = v - vo;
        const float cl = dlt < -clip ? -clip : (dlt > clip ? clip : dlt);      // (a NaN stays a NaN, as in torch.clamp)
        const float ec = (vo + cl) - rt;
        const float e2 = e * e, ec2 = ec * ec;
        const bool cut = fabsf(dlt) > clip && e2 < ec2;                        // (clip = +inf cuts nothing; a NaN v is not cut: it stays a NaN)
        const float loss = 0.5f * (cut ? ec2 : e2);
        const float dv = part && !cut ? e : 0.0f;                              // dL/dv
        const float err = rt - v;
        ab3 += dv;
        dms[lane] = dv;
        n_part += part ? 1u : 0u;
        n_cut += part && cut ? 1u : 0u;
        sum_l = part ? sum_l + loss : sum_l;
        sum_v = part ? sum_v + v : sum_v;
        sum_ret = part ? sum_ret + rt : sum_ret;
        sum_ret2 = part ? sum_ret2 + rt * rt : sum_ret2;
        sum_err2 = part ? sum_err2 + err * err : sum_err2;
        max_dv = part ? fmaxf(max_dv, fabsf(dlt)) : max_dv;
        if (value && part) value[i] = v;
        ppo_lds_order();

        // ---- dW3 += dv^T h2 (lane j: column j) ----
#pragma unroll 4
        for (int r = 0; r < kPpoBlock; ++r) aW3 = fmaf(dms[r], h2s[lane * S + r], aW3);
        ppo_lds_order();

        // ---- lane = row: dz2 over h2 in place, dh1 = W2^T dz2 ----
        float dh1[H];
#pragma unroll
        for (int c = 0; c < H; ++c) dh1[c] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
            pol_wptr row = w + O::W2 + j * H;
            const float dh2 = w[O::W3 + j] * dv;
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

    // ---- the workgroup's partial row: [WORDS] gradient sums, then n, sum L, cut, sum v, sum ret, sum ret^2, sum (ret - v)^2, max |v - v_old| ----
    float* const P = scratch + (size_t)blockIdx.x * (size_t)(O::WORDS + ATC_PPO_VALUE_STATS);
#pragma unroll
    for (int c = 0; c < IN; ++c) P[O::W1 + lane * IN + c] = aW1[c];
    P[O::B1 + lane] = ab1;
#pragma unroll
    for (int c = 0; c < H; ++c) P[O::W2 + lane * H + c] = aW2[c];
    P[O::B2 + lane] = ab2;
    P[O::W3 + lane] = aW3;
    // the per-lane sums, folded over the 64 lanes in lane order by lanes 0 .. 7, one word each: db3 first, then the statistics
    ppo_lds_order();
    dms[lane] = ab3;
    ppo_lds_order();
    if (lane == 0) {
        double s = 0.0;
        for (int l = 0; l < kPpoBlock; ++l) s += (double)dms[l];
        P[O::B3] = (float)s;
    }
    ppo_lds_order();
    dms[ATC_PPO_VSTAT_N * S + lane] = __uint_as_float(n_part);
    dms[ATC_PPO_VSTAT_LOSS * S + lane] = sum_l;
    dms[ATC_PPO_VSTAT_CUT * S + lane] = __uint_as_float(n_cut);
    dms[ATC_PPO_VSTAT_V * S + lane] = sum_v;
    dms[ATC_PPO_VSTAT_RET * S + lane] = sum_ret;
    dms[ATC_PPO_VSTAT_RET2 * S + lane] = sum_ret2;
    dms[ATC_PPO_VSTAT_ERR2 * S + lane] = sum_err2;
    dms[ATC_PPO_VSTAT_DV_MAX * S + lane] = max_dv;
    ppo_lds_order();
    if (lane < ATC_PPO_VALUE_STATS) {
        float word;
        if (lane == ATC_PPO_VSTAT_N || lane == ATC_PPO_VSTAT_CUT) {        // counts: exact, kept as integer bit patterns
            uint32_t n = 0u;
            for (int l = 0; l < kPpoBlock; ++l) n += __float_as_uint(dms[lane * S + l]);
            word = __uint_as_float(n);
        } else if (lane == ATC_PPO_VSTAT_DV_MAX) {
            float m = 0.0f;
            for (int l = 0; l < kPpoBlock; ++l) m = fmaxf(m, dms[lane * S + l]);
            word = m;
        } else {
            double s = 0.0;
            for (int l = 0; l < kPpoBlock; ++l) s += (double)dms[lane * S + l];
            word = (float)s;
        }
        P[O::WORDS + lane] = word;
    }
}

// k_ppo_grad_reduce with the critic's statistics (two counts, five means, one maximum; k_ppo_grad_reduce's cases are the policy's words):
// one lane per word of grad and of stats, the G partial rows in the order of g, in float64, rounded once; the division by n last
__global__ void __launch_bounds__(kPpoReduceBlock)
k_ppo_value_grad_reduce(int words, int G, const float* __restrict__ scratch, float* __restrict__ grad, float* __restrict__ stats) {
    const int wd = (int)(blockIdx.x * kPpoReduceBlock + threadIdx.x);
    if (wd >= words + ATC_PPO_VALUE_STATS) return;
    const size_t stride = (size_t)(words + ATC_PPO_VALUE_STATS);
    uint64_t n = 0ull;
    for (int g = 0; g < G; ++g) n += (uint64_t)__float_as_uint(scratch[(size_t)g * stride + (size_t)(words + ATC_PPO_VSTAT_N)]);
    const float nf = (float)n;
    const int q = wd - words;
    float out = 0.0f;
    if (q == ATC_PPO_VSTAT_N) {
        out = nf;
    } else if (q == ATC_PPO_VSTAT_CUT) {
        uint64_t c = 0ull;
        for (int g = 0; g < G; ++g) c += (uint64_t)__float_as_uint(scratch[(size_t)g * stride + (size_t)wd]);
        out = n ? (float)c / nf : 0.0f;
    } else if (q == ATC_PPO_VSTAT_DV_MAX) {
        float m = 0.0f;
        for (int g = 0; g < G; ++g) m = fmaxf(m, scratch[(size_t)g * stride + (size_t)wd]);
        out = n ? m : 0.0f;
    } else {                                // a word of grad, or one of the five means
        double s = 0.0;
        for (int g = 0; g < G; ++g) s += (double)scratch[(size_t)g * stride + (size_t)wd];
        const float v = (float)s;
        out = n ? v / nf : 0.0f;
    }
    if (q < 0) grad[wd] = out;
    else stats[q] = out;
}

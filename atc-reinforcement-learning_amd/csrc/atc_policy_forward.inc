// atc_policy_forward.inc — the decisions of the packed policy outside a rollout (include/atc_step.h: atc_policy_forward): k_policy_forward<KT>.
// Included by atc_step.hip behind atc_value.inc.
//   k_value_forward's shape with the policy's three-row head: LANE = ROW, 256 rows per workgroup, no LDS, no activation in memory; weights
//   through the constant address space at wave-uniform indices (scalar loads), the base pointer through the launch's opaque zero as in
//   policy_decide.  The MLP is evaluated ONCE per row; the S draws are a loop behind it that keeps mu in three registers.
//   THE TRUNK IS A COPY of policy_decide's text (atc_policy.inc), operation for operation — layer 1 as an fmaf chain from the bias, in
//   float64 where the WAVEFRONT (64 consecutive rows, row 0 first) holds an input above 4 in magnitude or a NaN; layer 2 in four partial
//   sums; the head folded into layer 2's loop — and not a call of it: policy_decide draws once and is inlined into the rollout kernels,
//   whose machine code stays as it is (DESIGN.md section 3p, 3s).  policy_z, mix64 and plan_draw_clamp are called as they are.  The file is
//   built with -ffp-contract=off: a row whose wavefront takes the same layer-1 form in both kernels gets the same bits in both.
//   No MFMA path: it would be another rounding of the same sums.  All stores are plain vector stores.
constexpr int kPolFwdBlock = 256;
// wavefronts per SIMD the kernel is register-budgeted for: k_value_forward's reasoning (64 h1 words and the input row live through layer 1):
// 3, and 2 with K = 4, whose 38 inputs in float32 and float64 next to h1 do not fit 168 registers.  -DATC_POLICY_FWD_WAVES=n: A/B builds.
#ifndef ATC_POLICY_FWD_WAVES
#define ATC_POLICY_FWD_WAVES 3
#endif

struct PolicyFwdDraw {
    uint64_t seed;
    uint32_t decision0;
    uint32_t dstride;    // decisions per sample: ceil(R / P)
    uint32_t P;          // rows per decision, 1 .. R
    int S;               // samples, 1 .. ATC_POLICY_FWD_MAX_SAMPLES
    uint32_t flags;      // ATC_POLICY_DETERMINISTIC
};

template <int KT>
__global__ void __launch_bounds__(kPolFwdBlock, KT == 4 && ATC_POLICY_FWD_WAVES > 2 ? 2 : ATC_POLICY_FWD_WAVES)
k_policy_forward(int R, const float* __restrict__ w_arg, const float* __restrict__ obs_rows, const float* __restrict__ traffic, PolicyFwdDraw dr,
                 float* __restrict__ mean, float* __restrict__ action, float* __restrict__ flown, float* __restrict__ logp) {
    constexpr int IN = ATC_POLICY_TRAFFIC_IN(KT), H = ATC_POLICY_HIDDEN;
    typedef PolOff<IN> O;
    const int zk = opaque_zero();
    pol_wptr w = (pol_wptr)(uintptr_t)w_arg;
    asm volatile("" : "+s"(w) : "s"(zk));
    const long long i = (long long)blockIdx.x * kPolFwdBlock + threadIdx.x;
    const bool have = i < (long long)R;
    float x[IN];
#pragma unroll
    for (int c = 0; c < IN; ++c) x[c] = 0.0f;
    if (have) {
        const float* o = obs_rows + (size_t)i * ATC_OBS_DIM;
#pragma unroll
        for (int c = 0; c < ATC_OBS_DIM; ++c) x[c] = o[c];
        if constexpr (KT > 0) {
            const float* t = traffic + (size_t)i * (size_t)(KT * ATC_TRAFFIC_DIM);
#pragma unroll
            for (int r = 0; r < KT; ++r)
#pragma unroll
                for (int c = 0; c < 7; ++c) x[ATC_OBS_DIM + 7 * r + c] = t[r * ATC_TRAFFIC_DIM + c];   // word 7 (the slot) is not read
        }
    }
    // ---- the trunk: policy_decide's, in its operation order ----
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
    for (int j = 0; j < H; ++j) h1[j] = tanhf(h1[j]);
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
#pragma unroll
        for (int c = 0; c < 3; ++c) mu[c] = fmaf(w[O::W3 + c * H + j], h2, mu[c]);
    }
    if (!have) return;   // (behind the trunk: the wavefront's choice of layer 1 is made with every lane present)
    const size_t r = (size_t)i, rows = (size_t)(uint32_t)R;
    if (mean) {
        float* m = mean + r * 3u;
        m[0] = mu[0]; m[1] = mu[1]; m[2] = mu[2];
    }
    if (!(action || flown || logp)) return;
    if (dr.flags & ATC_POLICY_DETERMINISTIC) {   // the rollout's rule: action = mean, logp = 0 (S == 1: the host refuses any other)
        if (action) {
            float* a = action + r * 3u;
            a[0] = mu[0]; a[1] = mu[1]; a[2] = mu[2];
        }
        if (flown) {
            float* a = flown + r * 3u;
            a[0] = plan_draw_clamp(mu[0]); a[1] = plan_draw_clamp(mu[1]); a[2] = plan_draw_clamp(mu[2]);
        }
        if (logp) logp[r] = 0.0f;
        return;
    }
    // ---- the S draws: policy_decide's key with decision = decision0 + s ceil(R / P) + r / P (modulo 2^32) and i = r % P ----
    const uint32_t rd = (uint32_t)i / dr.P, ri = (uint32_t)i - rd * dr.P;
    uint32_t decision = dr.decision0 + rd;
#pragma unroll 1
    for (int s = 0; s < dr.S; ++s, decision += dr.dstride) {
        const uint64_t key = mix64(mix64(dr.seed ^ (uint64_t)decision) ^ (uint64_t)ri);
        float u[3], lp = 0.0f;
#pragma unroll
        for (uint32_t c = 0; c < 3u; ++c) {
            const float ls = w[O::LOGSTD + c];
            const float z = policy_z(key, c);
            u[c] = mu[c] + expf(ls) * z;
            lp += -0.5f * (z * z) - ls;
        }
        const size_t at = (size_t)s * rows + r;
        if (action) {
            float* a = action + at * 3u;
            a[0] = u[0]; a[1] = u[1]; a[2] = u[2];
        }
        if (flown) {   // (a NaN gives -1)
            float* a = flown + at * 3u;
            a[0] = plan_draw_clamp(u[0]); a[1] = plan_draw_clamp(u[1]); a[2] = plan_draw_clamp(u[2]);
        }
        if (logp) logp[at] = lp - ATC_POL_LOGP_C;
    }
}
